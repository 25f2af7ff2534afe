// lhip_infotag.h -- the Info/LAME tag frame (extension { infoTag }): what the blob says about it (InfoTagCfg), the totals a stream keeps on the host
// (TagTotals: frames, audio bytes, running music CRC, seek-table bag, padding), the host's CRC arithmetic, and the frame itself.
// Host code only; nothing here reaches a kernel (Tables does not change: an untagged stream's kernels get the arguments they always got).
// Part of lhip_api.cpp's one translation unit (included there, in the order the definitions need).
//
// Layout: the public Xing / LAME tag format as LAME 3.98 writes it for CBR (VBRTag.js:830-960, 576-804) -- a frame of the stream's own header
// (padding 0, mode_ext 0) whose body starts where the side information would end (two bytes earlier in a protected stream, where the format
// places it): "Info", flags 0xF, frames, bytes (audio + this frame), 100 seek points, quality, "LAME3.98r", method, lowpass, peak and the two
// ReplayGain fields (peak and audiophile zero: the reference has no decoder, and LAME writes no album gain; the radio field is zero too unless the stream was
// built with { replayGain }: then it is the reference's encoding of the track gain the device analysed, lhip_gain.h), flags, bitrate, delay and padding (12 bits each),
// misc, one zero byte, preset, music length, music CRC, and the CRC-16 of every byte in front of that last field (190 of them in an
// unprotected MPEG-1 two-channel frame, the number the format's description names).
#pragma once
// what a blob built with { infoTag } carries (tables.js); on == 0: a blob without the option
struct InfoTagCfg {
    int on = 0, size = 0;       // size: bytes of the tag frame = floor((version + 1) * 72000 * brate / out_samplerate), LAME's integer division
    int quality = 0, method = 0, lowpass = 0, flags = 0, misc = 0, preset = 0, delay = 0;
    uint8_t version[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
};
enum { TAG_BODY_BYTES = 156, TAG_MAX_FRAME = 2880, TAG_TOC_BAG = 400 };      // LAMEHEADERSIZE; MAXFRAMESIZE (VBRTag.js:55-75)

// ---- the music CRC on the host: CRC-16, reflected polynomial 0xA001, preset 0 (k_crc.h has the device's form) ----
struct Crc16rTable { uint16_t v[256]; };
static const Crc16rTable& crc16r_table() {
    static const Crc16rTable t = []() {
        Crc16rTable r;
        for (int i = 0; i < 256; i++) { uint32_t c = (uint32_t)i; for (int b = 0; b < 8; b++) c = (c & 1) ? (c >> 1) ^ 0xA001u : c >> 1; r.v[i] = (uint16_t)c; }
        return r;
    }();
    return t;
}
static uint32_t crc16r_host(const uint8_t* p, size_t n, uint32_t crc = 0) {
    const Crc16rTable& t = crc16r_table();
    for (size_t i = 0; i < n; i++) crc = (crc >> 8) ^ t.v[(crc ^ p[i]) & 0xff];
    return crc;
}
// a * b mod the polynomial (reflected: bit 15 = x^0)
static uint32_t crc16r_mul(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 0; i < 16; i++) { r = (r >> 1) ^ ((r & 1) ? 0xA001u : 0u); if ((b >> i) & 1) r ^= a; }
    return r;
}
// crc(A ++ B) from crc(A), crc(B) and |B|: crc(A) x^(8 |B|) + crc(B); the power by square-and-multiply
static uint32_t crc16r_append(uint32_t crc_a, uint32_t crc_b, int64_t len_b) {
    if (crc_a) {
        uint32_t pw = 0x8000u, sq = 0x0080u;                    // x^0; x^8
        for (int64_t e = len_b; e > 0; e >>= 1) { if (e & 1) pw = crc16r_mul(pw, sq); sq = crc16r_mul(sq, sq); }
        crc_a = crc16r_mul(crc_a, pw);
    }
    return crc_a ^ crc_b;
}
// ISO 11172-3 CRC-16 (polynomial 0x8005, preset 0xffff, MSB first) of a protected frame's header bytes 2, 3 and side information
static uint32_t tag_iso_crc(const uint8_t* f, int sideinfo_len) {
    uint32_t crc = 0xffff;
    auto byte = [&](uint8_t b) { for (int i = 7; i >= 0; i--) { const uint32_t top = ((crc >> 15) & 1) ^ ((b >> i) & 1u); crc = (crc << 1) & 0xffff; if (top) crc ^= 0x8005; } };
    byte(f[2]); byte(f[3]);
    for (int i = 6; i < sideinfo_len; i++) byte(f[i]);
    return crc;
}

// ---- per-stream totals ----
// The seek-table bag is LAME's (VBRTag.js:146-185, with the integer halving of the C original): at most 400 running bitrate sums, one entry
// every `want` frames; when the bag is full every second entry is kept and `want` doubles.
struct TagTotals {
    int64_t frames = 0, bytes = 0;      // audio frames and bytes so far (the placeholder is neither)
    uint32_t crc = 0;                   // music CRC so far
    double padding = -1;                // gfp.encoder_padding, set by the flush (Lame.js:1409-1412)
    bool placed = false;                // the placeholder has been handed out (with the stream's first call)
    bool flushed = false, moved = false;       // moved: lhip_seek / lhip_state_set put the stream somewhere the totals do not describe
    int64_t sum = 0, seen = 0, want = 1; int pos = 0;
    int64_t bag[TAG_TOC_BAG];
};
// F frames of `kbps` each: one step per bag entry they complete, not per frame (in CBR every frame adds the same bitrate)
static void tag_toc_add(TagTotals& v, int64_t F, int kbps) {
    while (F > 0) {
        const int64_t need = v.want - v.seen;
        if (F < need) { v.sum += F * kbps; v.seen += F; return; }
        v.sum += need * kbps; F -= need;
        v.bag[v.pos++] = v.sum; v.seen = 0;
        if (v.pos == TAG_TOC_BAG) {
            for (int i = 1; i < TAG_TOC_BAG; i += 2) v.bag[i / 2] = v.bag[i];
            v.want *= 2; v.pos /= 2;
        }
    }
}
static void tag_toc(const TagTotals& v, uint8_t* toc) {
    memset(toc, 0, 100);
    if (v.pos <= 0 || v.sum <= 0) return;
    for (int i = 1; i < 100; i++) {
        int idx = (int)((int64_t)i * v.pos / 100);
        if (idx > v.pos - 1) idx = v.pos - 1;
        const int64_t sp = 256 * v.bag[idx] / v.sum;
        toc[i] = (uint8_t)(sp > 255 ? 255 : sp);
    }
}
// one call's audio of one stream
static void tag_account(TagTotals& v, int64_t F, int64_t bytes, uint32_t crc_call, int kbps) {
    v.frames += F;
    v.crc = crc16r_append(v.crc, crc_call & 0xffff, bytes);
    v.bytes += bytes;
    tag_toc_add(v, F, kbps);
}

// ---- the frame ----
static void tag_header(const Tables& T, uint8_t* f) {
    const uint32_t h = ((T.out_samplerate < 16000 ? 0xffeu : 0xfffu) << 20) | ((uint32_t)T.version << 19) | (1u << 17) | ((T.error_protection ? 0u : 1u) << 16) |
                       ((uint32_t)T.bitrate_index << 12) | ((uint32_t)T.samplerate_index << 10) | (0u << 9) | ((uint32_t)T.extension << 8) |
                       ((uint32_t)T.mode << 6) | (0u << 4) | ((uint32_t)T.copyright << 3) | ((uint32_t)T.original << 2) | (uint32_t)T.emphasis;
    f[0] = (uint8_t)(h >> 24); f[1] = (uint8_t)(h >> 16); f[2] = (uint8_t)(h >> 8); f[3] = (uint8_t)h;
}
// what the stream's first call hands out: a valid header, then zeros (LAME's contract: the frame is overwritten once the stream is complete)
static void tag_placeholder(const Tables& T, const InfoTagCfg& G, uint8_t* f) {
    memset(f, 0, (size_t)G.size);
    tag_header(T, f);
    if (T.error_protection) { const uint32_t c = tag_iso_crc(f, T.sideinfo_len); f[4] = (uint8_t)(c >> 8); f[5] = (uint8_t)c; }
}
static void tag_write(const Tables& T, const InfoTagCfg& G, const TagTotals& v, uint8_t* f, uint32_t radio_gain = 0) {
    memset(f, 0, (size_t)G.size);
    tag_header(T, f);
    int p = T.sideinfo_len - (T.error_protection ? 2 : 0);
    auto be32 = [&](uint32_t x) { f[p++] = (uint8_t)(x >> 24); f[p++] = (uint8_t)(x >> 16); f[p++] = (uint8_t)(x >> 8); f[p++] = (uint8_t)x; };
    auto be16 = [&](uint32_t x) { f[p++] = (uint8_t)(x >> 8); f[p++] = (uint8_t)x; };
    const uint32_t total = (uint32_t)(v.bytes + G.size);
    f[p++] = 'I'; f[p++] = 'n'; f[p++] = 'f'; f[p++] = 'o';
    be32(0xF); be32((uint32_t)v.frames); be32(total);
    tag_toc(v, f + p); p += 100;
    be32((uint32_t)G.quality);
    memcpy(f + p, G.version, 9); p += 9;
    f[p++] = (uint8_t)G.method; f[p++] = (uint8_t)G.lowpass;
    be32(0); be16(radio_gain); be16(0);                          // peak signal amplitude (no decoder: zero), radio ReplayGain ({ replayGain } streams, else zero), audiophile (LAME writes none)
    f[p++] = (uint8_t)G.flags;
    f[p++] = (uint8_t)(T.brate >= 255 ? 255 : T.brate);
    const uint32_t delay = (uint32_t)G.delay & 0xfff, pad = (uint32_t)(v.padding < 0 ? 0 : (int64_t)v.padding) & 0xfff;      // (a fraction is cut as `>>` cuts it)
    f[p++] = (uint8_t)(delay >> 4); f[p++] = (uint8_t)((delay << 4) | (pad >> 8)); f[p++] = (uint8_t)pad;
    f[p++] = (uint8_t)G.misc; f[p++] = 0;
    be16((uint32_t)G.preset); be32(total); be16(v.crc & 0xffff);
    // the header CRC of a protected stream covers the side-information bytes the tag's first two characters now occupy; the tag's own CRC covers it in turn
    if (T.error_protection) { const uint32_t c = tag_iso_crc(f, T.sideinfo_len); f[4] = (uint8_t)(c >> 8); f[5] = (uint8_t)c; }
    be16(crc16r_host(f, (size_t)p));
}
