/* TEST TOOL (tests/test_wavpcm_cpu.py::test_bounds_under_asan): built with -fsanitize=address together with lhip_api.cpp as a simulation
 * (-DLHIP_HOSTSIM, and once more with -DLHIP_WAVESIM), so that every load and store of the g_ingest kernel body is checked.  Every input lies in a
 * heap block that ENDS with its last byte; in front of its first byte lie `misalign` bytes and 16 more, poisoned as far as AddressSanitizer can poison
 * (whole 8-byte granules: all of the piece in front of the window, and the first half of the head piece where misalign >= 8), so that a wide load of
 * the ragged head is seen like one past the tail.  The simulations' "device" pointers are host pointers, so the device entry reads these blocks
 * directly; lhip_debug_ingest lays its own copy out the same way and fills one block of exactly n floats per plane.
 * usage: wavpcm_bounds <tables blob of (2, 44100, 128)> */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sanitizer/asan_interface.h>
#include "lamejs_hip.h"

static uint32_t rnd_state = 12345u;
static uint32_t rnd(void) { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static int fail(const char* what, int a, int b, int c) { fprintf(stderr, "wavpcm_bounds: %s (%d, %d, %d): %s\n", what, a, b, c, lhip_last_error()); return 1; }

static float want_s24(const uint8_t* p) {
    int32_t v = (int32_t)((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16));
    if (v & 0x800000) v -= 0x1000000;
    return (float)v / 256.0f;
}

int main(int argc, char** argv) {
    static const int NS[] = {1, 2, 5, 15, 16, 17, 21, 1151, 1153};
    static const int SIX[] = {0, 1, 1152, 1153, 2305, 777};
    if (argc < 2) { fprintf(stderr, "usage: wavpcm_bounds <tables blob>\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    fseek(f, 0, SEEK_END);
    long tb = ftell(f);
    fseek(f, 0, SEEK_SET);
    void* tables = malloc((size_t)tb);
    if (fread(tables, 1, (size_t)tb, f) != (size_t)tb) return 2;
    fclose(f);
    long checks = 0;
    /* lhip_debug_ingest: S24, every misalignment, the lengths of the shapes test; mono, interleaved stereo, planar stereo; U8 at odd addresses */
    for (int type = LHIP_PCM_S24; type >= LHIP_PCM_U8; type -= 4) {
        const int bps = type == LHIP_PCM_S24 ? 3 : 1;
        for (size_t ni = 0; ni < sizeof NS / sizeof NS[0]; ni++)
            for (int mis = (type == LHIP_PCM_U8 ? 1 : 0); mis < 16; mis += (type == LHIP_PCM_U8 ? 2 : 1))
                for (int layout = 0; layout < 3; layout++) {
                    const int n = NS[ni], ch = layout ? 2 : 1;
                    const size_t nb = (size_t)n * bps * ch;
                    uint8_t* in = (uint8_t*)malloc(nb);
                    float* l = (float*)malloc((size_t)n * 4);
                    float* r = (float*)malloc((size_t)n * 4);
                    int64_t rej = -1;
                    for (size_t i = 0; i < nb; i++) in[i] = (uint8_t)rnd();
                    if (lhip_debug_ingest(type | (layout == 1 ? LHIP_PCM_INTERLEAVED : 0), ch, in, (size_t)n, (size_t)mis, l, ch == 2 ? r : NULL, &rej) != 0 || rej != 0) return fail("lhip_debug_ingest", n, mis, layout);
                    for (int i = 0; i < n; i++) {
                        const size_t el = layout == 1 ? 2 * (size_t)i : (size_t)i, er = layout == 1 ? 2 * (size_t)i + 1 : (size_t)n + i;
                        const float wl = type == LHIP_PCM_S24 ? want_s24(in + 3 * el) : (float)(((int)in[el] - 128) * 256);
                        if (l[i] != wl) return fail("left plane", n, mis, i);
                        if (ch == 2) { const float wr = type == LHIP_PCM_S24 ? want_s24(in + 3 * er) : (float)(((int)in[er] - 128) * 256); if (r[i] != wr) return fail("right plane", n, mis, i); }
                    }
                    free(in); free(l); free(r);
                    checks++;
                }
    }
    /* the encode entries: six streams of the batch test's lengths, S24, through the host entry and through the device entry (which reads the blocks in place) */
    const lhip_config cfg = {2, 44100, 128, -1};
    for (int entry = 0; entry < 2; entry++)
        for (int layout = 1; layout < 3; layout++)
            for (int mis = 0; mis < 16; mis += 5) {
                lhip_stream* s[6]; const void* lp[6]; const void* rp[6]; size_t ns[6], cap[6]; uint8_t* out[6]; int64_t wr[6]; uint8_t* blk[12];
                for (int i = 0; i < 6; i++) {
                    if (lhip_create(&cfg, tables, (size_t)tb, &s[i]) != 0) return fail("lhip_create", i, 0, 0);
                    const size_t n = (size_t)SIX[i], plane = n * 3 * (layout == 1 ? 2 : 1);
                    ns[i] = n; cap[i] = lhip_max_output_bytes(s[i], n); out[i] = (uint8_t*)malloc(cap[i]);
                    for (int k = 0; k < 2; k++) {
                        blk[2 * i + k] = (uint8_t*)malloc(16 + (size_t)mis + plane);
                        if ((uintptr_t)blk[2 * i + k] & 15) return fail("malloc alignment", i, k, mis);
                        ASAN_POISON_MEMORY_REGION(blk[2 * i + k], 16 + (size_t)(mis & ~7));
                        for (size_t b = 0; b < plane; b++) blk[2 * i + k][16 + mis + b] = (b % 3 == 2) ? (uint8_t)((rnd() & 1) ? 0xff : 0x00) : (uint8_t)rnd();      /* within Int16 after the division */
                    }
                    lp[i] = blk[2 * i] + 16 + mis; rp[i] = layout == 1 ? NULL : blk[2 * i + 1] + 16 + mis;
                }
                const int fmt = LHIP_PCM_S24 | (layout == 1 ? LHIP_PCM_INTERLEAVED : 0);
                const int rc = entry == 0 ? lhip_encode_batch_pcm(s, 6, fmt, lp, rp, ns, out, cap, wr) : lhip_encode_batch_device_pcm(s, 6, fmt, lp, rp, ns, out, cap, wr, 1);
                if (rc != 0) return fail("encode batch", entry, layout, mis);
                uint32_t paths = 0;
                lhip_debug_last_paths(&paths);
                if (entry == 1 && !(paths & LHIP_PATH_INGEST)) return fail("the device entry did not launch g_ingest", entry, layout, mis);
                /* one stream on its own: lhip_encode_pcm (a small call: the host converts the caller's block itself) */
                uint8_t tail[8192];
                if (lhip_encode_pcm(s[5], fmt, lp[5], rp[5], ns[5], tail, sizeof tail) < 0) return fail("lhip_encode_pcm", entry, layout, mis);
                for (int i = 0; i < 6; i++) { lhip_destroy(s[i]); free(out[i]); for (int k = 0; k < 2; k++) { ASAN_UNPOISON_MEMORY_REGION(blk[2 * i + k], 16 + (size_t)mis); free(blk[2 * i + k]); } }
                checks++;
            }
    free(tables);
    printf("wavpcm_bounds OK: %ld checks\n", checks);
    return 0;
}
