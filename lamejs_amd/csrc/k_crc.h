// k_crc.h -- the music CRC of the Info tag (extension { infoTag }; BitStream.js:927, VBRTag.js:100-141): the CRC-16 with the reflected polynomial
// 0xA001, register preset to 0, no final XOR, over every audio byte a stream has put out.  The bytes of a call are in HBM when its last writer
// (g_bits, g_frame, g_resv_stream, g_resv_flush) is done; kb_out_crc reads them there once.
//
// With a zero preset the register is linear over GF(2) with no affine term: crc(A ++ B) = crc(A) x^(8 |B|) + crc(B) mod the polynomial, and zero
// bytes in front of a message change nothing.  So the bytes of a stream's call split freely:
//   lane       16 bytes in one load, reduced byte by byte (crcr_byte: shifts and XORs, no table)
//   wave       lane l's remainder times the constant x^(8 16 (63 - l)), added with wave_xor -- the pattern of bits_crc (k_bits.h)
//   workgroup  one wave walks a SPAN of CRC_SPAN_BYTES from its front to its rear, remainder times x^(8 1024) per step (Horner)
//   stream     kb_crc_fold: the span remainders, each times x^(8 bytes behind the span) -- constants again, since spans have one size
// Everything is addressed by its distance FROM THE END of the stream's bytes: a span, a wave's 1024 bytes and a lane's 16 then lie at fixed
// distances whatever the start address and the length are (frames are 417 / 418 bytes; the second stream of a batch starts at an odd address),
// and what would lie in front of the first byte is read as zero -- the lane that straddles the start takes its bytes one by one, nothing else differs.
// Reflected representation: bit 15 of a 16-bit value is the coefficient of x^0, bit 0 that of x^15 (the register's own layout).
#pragma once
#include "lhip_defs.h"
#include "lhip_wave.h"

namespace lhip {

enum { CRCR_POLY = 0xA001, CRC_LANE_BYTES = 16, CRC_WAVE_BYTES = 64 * CRC_LANE_BYTES, CRC_SPAN_ITERS = 16, CRC_SPAN_BYTES = CRC_SPAN_ITERS * CRC_WAVE_BYTES };

// one stream's bytes of the call: `n` of them from `base`, or -- the bit reservoir, where only the device knows -- *n_dev; its span remainders start at part0
struct CrcDesc { const uint8_t* base; int64_t n; const int32_t* n_dev; int32_t part0, nparts; };

constexpr uint32_t crcr_mulx_c(uint32_t v) { return (v >> 1) ^ ((v & 1) ? (uint32_t)CRCR_POLY : 0u); }
constexpr uint32_t crcr_mul_c(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 0; i < 16; i++) { r = crcr_mulx_c(r); if ((b >> i) & 1) r ^= a; }
    return r;
}
struct CrcrPow {
    uint16_t lane[64];          // x^(8 16 (63 - l))
    uint16_t span[64];          // x^(8 SPAN l)
    uint16_t x_wave, x_span64;  // x^(8 1024), x^(8 SPAN 64)
};
constexpr CrcrPow crcr_pow() {
    CrcrPow t{};
    uint32_t x128 = 0x8000;                                       // x^0 ...
    for (int i = 0; i < 8 * CRC_LANE_BYTES; i++) x128 = crcr_mulx_c(x128);      // ... to x^(8 16)
    uint32_t r = 0x8000;
    for (int l = 63; l >= 0; l--) { t.lane[l] = (uint16_t)r; r = crcr_mul_c(r, x128); }
    t.x_wave = (uint16_t)r;
    uint32_t xs = r;
    for (int i = 1; i < CRC_SPAN_ITERS; i <<= 1) xs = crcr_mul_c(xs, xs);          // (x^(8 1024))^16
    static_assert(CRC_SPAN_ITERS == 16, "x_span is x_wave squared four times");
    r = 0x8000;
    for (int l = 0; l < 64; l++) { t.span[l] = (uint16_t)r; r = crcr_mul_c(r, xs); }
    t.x_span64 = (uint16_t)r;
    return t;
}
// a * b mod the polynomial (a, b < 2^16, reflected)
LHIP_DEV uint32_t crcr_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        r = (r >> 1) ^ ((r & 1) ? (uint32_t)CRCR_POLY : 0u);
        if ((b >> i) & 1) r ^= a;
    }
    return r;
}
// The register after one more byte.  With t = (crc ^ b) & 0xff the eight shift-and-XOR steps of the bitwise form collapse, for THIS polynomial
// (x^16 + x^15 + x^2 + 1: three taps), into the parity of t at the taps 0xC001 and t at two shifts -- nine operations for eight bits, no table.
LHIP_DEV uint32_t crcr_byte(uint32_t crc, uint32_t b) {
    const uint32_t t = (crc ^ b) & 0xffu;
    const uint32_t par = (uint32_t)__builtin_popcount(t) & 1u;
    return (crc >> 8) ^ (par ? 0xC001u : 0u) ^ (t << 6) ^ (t << 7);
}
// sixteen bytes from any address, oldest first
LHIP_DEV uint32_t crcr_block16(const uint8_t* p) {
    uint32_t w[4];
    __builtin_memcpy(w, p, 16);                                  // one wide load (the address need not be aligned)
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) c = crcr_byte(c, (w[k >> 2] >> (8 * (k & 3))) & 0xffu);
    return c;
}
LHIP_DEV int64_t crc_len(const CrcDesc& d) { return d.n_dev ? (int64_t)*d.n_dev : d.n; }
// workgroup b of the launch -> its stream: the last one whose part0 is <= b (part0 ascends; nstreams >= 1, 0 <= b < the sum of nparts)
LHIP_DEV int crc_find_stream(const CrcDesc* D, int nstreams, int b) {
    int lo = 0, hi = nstreams - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (D[mid].part0 <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// span `span` of stream `stream` (the bytes at distances (span SPAN, (span + 1) SPAN] from the end); one wave
LHIP_DEV void kb_out_crc(const CrcDesc* D, int stream, int span, int lane, uint32_t* partial) {
    constexpr CrcrPow pw = crcr_pow();
    const CrcDesc d = D[stream];
    const int64_t n = crc_len(d);
    if (span >= d.nparts || (int64_t)span * CRC_SPAN_BYTES >= n) return;      // nothing of the stream lies this far from its end (wave-uniform)
    const uint8_t* end = d.base + n;
    uint32_t R = 0;
    for (int t = 0; t < CRC_SPAN_ITERS; t++) {
        const int64_t hi = (int64_t)span * CRC_SPAN_BYTES + (int64_t)(CRC_SPAN_ITERS - t) * CRC_WAVE_BYTES;      // distance of this step's first byte from the end
        if (hi - CRC_WAVE_BYTES >= n) continue;                   // wholly in front of the first byte: zeros (R is still 0)
        uint32_t c = 0;
        for (int l = lane; l < 64; l += LHIP_NL) {                // (one trip on the device; the one-lane simulation walks the lanes)
            const int64_t d0 = hi - CRC_LANE_BYTES * l;           // distance of the lane's first byte
            uint32_t r = 0;
            if (d0 <= n) r = crcr_block16(end - d0);
            else if (d0 - CRC_LANE_BYTES < n) { for (int64_t k = n; k > d0 - CRC_LANE_BYTES; k--) r = crcr_byte(r, end[-k]); }      // the lane that straddles the start
            c ^= crcr_mul(r, pw.lane[l]);
        }
        c = (uint32_t)wave_xor((int)c);
        R = crcr_mul(R, pw.x_wave) ^ c;
    }
    if (lane == 0) partial[d.part0 + span] = R;
}
// a stream's span remainders into its CRC; one wave.  Lane l takes the spans l, l + 64, ... (Horner with x^(8 SPAN 64)), then its place x^(8 SPAN l).
LHIP_DEV void kb_crc_fold(const CrcDesc* D, int stream, int lane, const uint32_t* partial, uint32_t* out) {
    constexpr CrcrPow pw = crcr_pow();
    const CrcDesc d = D[stream];
    const int64_t n = crc_len(d);
    int64_t ns64 = (n + CRC_SPAN_BYTES - 1) / CRC_SPAN_BYTES;
    if (ns64 > d.nparts) ns64 = d.nparts;                         // (cannot happen: the host sized nparts for the call's upper bound)
    const int nspans = (int)ns64;
    uint32_t acc = 0;
    for (int l = lane; l < 64; l += LHIP_NL) {
        uint32_t a = 0;
        if (l < nspans)
            for (int j = l + 64 * ((nspans - 1 - l) / 64); j >= l; j -= 64) a = crcr_mul(a, pw.x_span64) ^ partial[d.part0 + j];
        acc ^= crcr_mul(a, pw.span[l]);
    }
    acc = (uint32_t)wave_xor((int)acc);
    if (lane == 0) out[stream] = acc;
}

}  // namespace lhip
