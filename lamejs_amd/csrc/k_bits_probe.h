// k_bits_probe.h -- TEST HOOK (lhip_debug_bits_probe): the bitstream formatter over caller-supplied frames.  Nothing of the formatter is restated here: the probe
// calls kb_bits and kb_bits_mw (k_bits.h) as the shipped kernels do, on a workspace that holds the caller's side records and spectra and nothing else -- record r
// is frame r of a "stream" of its own (StreamDesc r: fslot0 = -1, so k = r; the slot lag of a fresh stream), whose output goes to a window of the output buffer
// that is r bytes longer than a frame, so that where bits_copy_out placed the frame can be read off the buffer afterwards.  No shipped kernel calls anything in
// this file.  The record layouts are the ones include/lamejs_hip.h states (little-endian, natural alignment).
#pragma once
#include "k_bits.h"

namespace lhip {

enum { BITS_PROBE_FRAME_BYTES = 1448, BITS_PROBE_OUT_BYTES = 1464, BITS_PROBE_MAX_RECORDS = 8192, BITS_PROBE_SLACK = 16 };
// record in: GrSide side[GR * C] | int16 l3[GR * C][576]
struct BitsProbeOut { uint8_t bytes[BITS_PROBE_FRAME_BYTES]; int32_t nbytes, status; int64_t offset; };
static_assert(sizeof(BitsProbeOut) == BITS_PROBE_OUT_BYTES && sizeof(GrSide) == 464, "the record layouts of include/lamejs_hip.h");
// the kernel's one argument (g_bits_probe, lhip_probe.cpp); `grid` = the workgroups launched
struct BitsProbeArgs { Tables T; Workspace W; const StreamDesc* SD; int n, grid, form, pad_; };

}  // namespace lhip
