// Psychoacoustic model kernels (nspsytune), decomposed per SURVEY.md 3.4:
//   kb_psyA  : per (psy call, channel) -- everything that is a pure function of the PCM window:
//              fs/4 high-pass + sub-block peaks, 1024-pt and 3x256-pt windowed FHT, energies,
//              loudness, partition energies / tonality index, short-block spreading.
//   kb_scan  : per stream -- the two tiny recurrences (attack/block-type chain, ATH auto-adjust).
//   kb_psyB  : per psy call -- thresholds that need the scan results (additive masking with the
//              adjusted ATH, short-block limiting, sfb mapping, inter-channel masking).
// Behaviour follows reference PsyModel.js:1000-1383 (L3psycho_anal_ns), FFT.js:31-224 and
// Encoder.js:166-243 (adjust_ATH); line references are given at each step.
#pragma once
#include <type_traits>
#include "lhip_defs.h"
#include "lhip_wave.h"
#include "lhip_math.h"
#include "lhip_layout.h"
#include "k_psy_fht.h"     // the FHT butterflies and the padded LDS layout of a transform buffer
#include "k_psy_a.h"       // kb_psyA with its LDS record, psy_need_s / psy_need_f
#include "k_psy_scan.h"    // the per-stream scans: attack flags, block types, the ATH recurrence
#include "k_psy_b.h"       // kb_psyB with its LDS record and the mask_add tables
