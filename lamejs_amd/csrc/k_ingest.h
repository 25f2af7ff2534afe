// k_ingest.h -- sample types a WAV file stores (extension; lamejs_hip.h: LHIP_PCM_U8 .. LHIP_PCM_F64): kb_ingest turns a call's new samples into Float32
// planes with stride 1, in front of the call's first reader.  Behind the planes a call IS a Float32 planar call (StreamIO: f32 = 1, stride = 1), so
// no staging loop of the psychoacoustics, the filterbank or the frame program knows these types.
//
// A type is defined by the number the reference would find in its Float32 buffer (Lame.js:1506-1510) had the caller widened the samples:
//   U8    (b - 128) * 256                 exact
//   S24   v / 256                         exact: 24 significant bits
//   S32   (float)(v / 65536.0)            one rounding, to nearest even
//   F32N  x * 32768                       exact (a power of two) unless it overflows
//   F64N  (float)(x * 32768.0)            the product is exact, one rounding
//   F64   (float)x                        one rounding
// The float types carry the contract of Float32 input behind the conversion: the value must be finite and within Tables::pcm_limit.  F64N / F64 are
// compared BEFORE the rounding (a double above the limit is refused even where it would round onto it; one just below it rounds onto it and is
// accepted); a refused sample is +0 in the plane and counted.  The integer types cannot leave the contract: 32768 at most, and pcm_limit >= 32768.
//
// Work split.  The elements of a call's source array (one plane, or the interleaved pair) are cut into STEPS of ING_STEP_BYTES; a wave takes ING_STEPS
// of them.  Per step the 16-byte pieces that cover the step's bytes -- at most 64, the source may start anywhere -- are loaded one per lane
// (lane i at window + 16 i: one wide load each) into LDS, where the elements, 3-byte ones that straddle two pieces included, are read back; a piece
// that is not wholly inside the array (the ragged head and tail) is taken byte by byte.  No load touches a byte outside [src, src + bytes), no store a
// float outside [dst, dst + n).  Interleaved two-channel input is split into its two planes in the same pass.
#pragma once
#include "lhip_defs.h"
#include "lhip_wave.h"

namespace lhip {

enum { ING_U8 = 4, ING_S24 = 8, ING_S32 = 12, ING_F32N = 16, ING_F64N = 20, ING_F64 = 24 };      // the sample types (format & ~INTERLEAVED) of lamejs_hip.h
enum { ING_PIECE = 16, ING_WINDOW = 64 * ING_PIECE, ING_STEP_BYTES = ING_WINDOW - ING_PIECE, ING_STEPS = 8 };
static_assert(ING_STEP_BYTES % 3 == 0 && ING_STEP_BYTES % 8 == 0, "a step holds whole elements of every type");

#ifdef LHIP_HOSTSIM
#define LHIP_HD static inline
#else
#define LHIP_HD static __host__ __device__ __forceinline__
#endif

LHIP_HD int ingest_bps(int type) { return type == ING_U8 ? 1 : type == ING_S24 ? 3 : (type == ING_F64N || type == ING_F64) ? 8 : 4; }
LHIP_HD bool ingest_is_float(int type) { return type >= ING_F32N; }

// one element at p -> the Float32 the encoder sees.  ALIGNED: p is a multiple of the element size (the kernel's reads of 4- and 8-byte elements)
template <bool ALIGNED> LHIP_HD float ingest_value(int type, const uint8_t* p, float limit, unsigned* bad) {
    switch (type) {
        case ING_U8: return (float)(((int)p[0] - 128) * 256);
        case ING_S24: {
            const uint32_t u = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
            return (float)((int32_t)(u << 8) >> 8) * (1.0f / 256.0f);
        }
        case ING_S32: {
            int32_t v;
            __builtin_memcpy(&v, ALIGNED ? __builtin_assume_aligned(p, 4) : (const void*)p, 4);
            return (float)((double)v * (1.0 / 65536.0));
        }
        case ING_F32N: {
            float x;
            __builtin_memcpy(&x, ALIGNED ? __builtin_assume_aligned(p, 4) : (const void*)p, 4);
            const float v = x * 32768.0f;
            if (!((v < 0 ? -v : v) <= limit)) { ++*bad; return 0.f; }
            return v;
        }
        default: {       // ING_F64N, ING_F64
            double x;
            __builtin_memcpy(&x, ALIGNED ? __builtin_assume_aligned(p, 8) : (const void*)p, 8);
            const double d = type == ING_F64N ? x * 32768.0 : x;
            if (!((d < 0 ? -d : d) <= (double)limit)) { ++*bad; return 0.f; }
            return (float)d;
        }
    }
}

// One stream's new samples of the call.  narr source arrays of nelem elements each: one (a single plane; the interleaved pair: inter = 1, 2 n
// elements, dst[e & 1][e >> 1]) or two (planar stereo: array a -> dst[a]).  The stream's workgroups are blk0 .. blk0 + narr * tiles - 1 of the launch.
struct IngestDesc { const uint8_t* src[2]; float* dst[2]; int64_t nelem, tiles; int32_t type, inter, narr, blk0; };

// the workgroups one source array of nelem elements takes
LHIP_HD int64_t ingest_tiles(int type, int64_t nelem) {
    const int64_t per = (int64_t)ING_STEPS * (ING_STEP_BYTES / ingest_bps(type));
    return (nelem + per - 1) / per;
}
// workgroup b of the launch -> its stream: the last one whose blk0 is <= b (blk0 ascends; a stream without samples has no workgroup)
LHIP_DEV int ingest_find_stream(const IngestDesc* D, int nstreams, int b) {
    int lo = 0, hi = nstreams - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (D[mid].blk0 <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// 16 bytes of a source array [lo, hi) at the 16-byte aligned address q into LDS: one wide load where the piece lies inside the array, else its bytes singly
LHIP_DEV void ingest_piece(uint8_t* dst, uintptr_t q, uintptr_t lo, uintptr_t hi) {
    if (q >= lo && q + ING_PIECE <= hi) { __builtin_memcpy(__builtin_assume_aligned(dst, 16), __builtin_assume_aligned((const void*)q, 16), ING_PIECE); return; }
    for (int k = 0; k < ING_PIECE; k++) if (q + k >= lo && q + k < hi) dst[k] = *(const uint8_t*)(q + k);
}
// tile `tile` (0 <= tile < narr * tiles) of stream `stream`; one wave, `lds`: ING_WINDOW bytes, 16-byte aligned.  Returns the wave's refused samples (wave-uniform).
LHIP_DEV unsigned kb_ingest(const IngestDesc* D, int stream, int64_t tile, int lane, uint8_t* lds, float limit) {
    const IngestDesc d = D[stream];
    const int type = d.type, bps = ingest_bps(type), ept = ING_STEP_BYTES / bps;
    const int arr = d.tiles > 0 ? (int)(tile / d.tiles) : 0;
    if (arr >= d.narr) return 0;                                     // (cannot happen: the host sized the grid)
    const int64_t t = tile - (int64_t)arr * d.tiles;
    const uint8_t* src = arr ? d.src[1] : d.src[0];
    const uintptr_t lo = (uintptr_t)src, hi = lo + (uintptr_t)d.nelem * (uintptr_t)bps;
    float* const plane = arr ? d.dst[1] : d.dst[0];
    unsigned bad = 0;
    for (int it = 0; it < ING_STEPS; it++) {
        const int64_t e0 = (t * ING_STEPS + it) * ept;
        if (e0 >= d.nelem) break;                                    // wave-uniform
        const int ne = d.nelem - e0 < ept ? (int)(d.nelem - e0) : ept;
        const uintptr_t tb = lo + (uintptr_t)e0 * (uintptr_t)bps, te = tb + (uintptr_t)ne * (uintptr_t)bps;
        const uintptr_t w0 = tb & ~(uintptr_t)(ING_PIECE - 1);
        const int npieces = (int)((te - w0 + ING_PIECE - 1) / ING_PIECE);      // <= 64: 15 + ING_STEP_BYTES bytes at most
        wave_sync();                                                 // the step before has been read
        for (int p = lane; p < npieces; p += LHIP_NL) ingest_piece(lds + ING_PIECE * p, w0 + (uintptr_t)ING_PIECE * p, lo, hi);
        wave_sync();
        const int off0 = (int)(tb - w0);
        for (int k = lane; k < ne; k += LHIP_NL) {
            const float v = ingest_value<true>(type, lds + off0 + k * bps, limit, &bad);
            const int64_t e = e0 + k;
            if (d.inter) { float* q = (e & 1) ? d.dst[1] : d.dst[0]; q[e >> 1] = v; }
            else plane[e] = v;
        }
    }
    return (unsigned)wave_sum((int)bad);
}

// the host's form of the same conversion (a small host call is converted while its pinned block is filled): n samples per channel, nch channels
static inline unsigned ingest_host(int type, const void* left, const void* right, size_t n, int nch, bool inter, float* dst0, float* dst1, float limit) {
    const int bps = ingest_bps(type);
    unsigned bad = 0;
    const uint8_t* l = (const uint8_t*)left;
    if (inter && nch == 2) {
        for (size_t i = 0; i < n; i++) {
            dst0[i] = ingest_value<false>(type, l + (2 * i) * (size_t)bps, limit, &bad);
            dst1[i] = ingest_value<false>(type, l + (2 * i + 1) * (size_t)bps, limit, &bad);
        }
        return bad;
    }
    for (size_t i = 0; i < n; i++) dst0[i] = ingest_value<false>(type, l + i * (size_t)bps, limit, &bad);
    if (nch == 2 && dst1) { const uint8_t* r = (const uint8_t*)(right ? right : left); for (size_t i = 0; i < n; i++) dst1[i] = ingest_value<false>(type, r + i * (size_t)bps, limit, &bad); }
    return bad;
}

}  // namespace lhip
