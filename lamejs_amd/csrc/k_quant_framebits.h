// k_quant_framebits.h -- the size of a frame in bits and its padding bit.  The frame program (k_quant_frame.h) and the bit packer (k_bits.h) both
// need them, and the packer needs nothing else of the search: this file depends on the definitions and the layout alone.
#pragma once
#include "lhip_defs.h"
#include "lhip_math.h"
#include "lhip_layout.h"
namespace lhip {
LHIP_DEV int frame_bits_of(const Tables& T, int padding) {
    return 8 * js_toint32((double)((T.version + 1) * 72000 * T.brate) / T.out_samplerate + padding);
}

// padding bit of the k-th frame of this batch (Encoder.js:442-446): slot_lag is decremented by frac_SpF
// every frame and wrapped by out_samplerate whenever it drops below zero
LHIP_DEV int frame_padding(const Tables& T, const StreamDesc& sd, int k) {
    if (T.frac_SpF == 0) return 0;
    // value held before frame k:  lag0 - k*frac  (mod out_samplerate), representative in [0, out_samplerate)
    int64_t m = ((int64_t)sd.slot_lag - (int64_t)k * T.frac_SpF) % T.out_samplerate;
    if (m < 0) m += T.out_samplerate;
    return (m - T.frac_SpF) < 0 ? 1 : 0;
}
}  // namespace lhip
