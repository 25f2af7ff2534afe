/*
 * TEST INFRASTRUCTURE -- public interface of the CPU oracle (see lame_oracle.c).
 * Mirrors the reference's stream API: create(config blob) / encode(Int16 PCM) / flush.
 */
#ifndef LAME_ORACLE_H
#define LAME_ORACLE_H
#include <stdint.h>
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef struct lo_enc lo_enc;
/* blob: LHTB table blob produced by lamejs_amd/js/tables.js (copied; caller may free) */
lo_enc* lo_create(const void* blob, size_t nbytes);
void lo_destroy(lo_enc* e);
/* appends whole MP3 frames completed by these samples; returns bytes written, -1 if out too small */
long lo_encode(lo_enc* e, const int16_t* left, const int16_t* right, size_t nsamples, uint8_t* out, size_t cap);
long lo_flush(lo_enc* e, uint8_t* out, size_t cap);
int lo_frame_bytes_max(const lo_enc* e);
/* stage-level taps of the most recent frame (struct lo_tap in lo_common.h) */
void lo_enable_tap(lo_enc* e);
const void* lo_get_tap(const lo_enc* e);
size_t lo_tap_size(void);
/* the quantization probe (lo_quant.c): n records of 4144 bytes in, n of 6352 bytes out, with e's tables; e's stream state is left as it was */
void lo_quant_probe(lo_enc* e, const void* in, size_t n, void* out);
/* the bitstream probe (lame_oracle.c): n frames in (mode_gr * channels side records of 464 bytes, then as many signed int16 spectra of 576 lines: the layout of the
 * library's lhip_debug_bits_probe), n records of 1464 bytes out (frame bytes[1448], int32 nbytes, int32 status, int64 offset); record k is formatted as frame k of
 * a fresh stream by lo_format_frame.  status -1: the record does not fill its frame exactly (where the encoder's path aborts).  No bit reservoir; e's stream
 * state is left as it was.  Returns 0, or -1 for a reservoir configuration. */
int lo_bits_probe(lo_enc* e, const void* in, size_t n, void* out);
#ifdef __cplusplus
}
#endif
#endif
