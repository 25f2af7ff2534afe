// CBR quantization / noise-shaping loop as a wave program: one 64-lane wavefront owns one frame
// and runs granule 0 (all channels) then granule 1, exactly as the reference's
// CBRNewIterationLoop.iteration_loop does (CBRNewIterationLoop.js:25-90).  Inside a
// granule-channel the *control flow* of the reference (Quantize.js outer_loop 871-1052,
// bin_search_StepSize 322-381, balance_noise 793-846, ...) is executed uniformly by all lanes,
// while every loop over the 576 spectral lines / the scalefactor bands is spread over the lanes:
//   - quantize x^(3/4) lines (Takehiro.js:102-314): five pairs per lane, per-band decisions as ballots
//   - Huffman bit counting (Takehiro.js:319-628): region maxima and packed length sums by
//     integer wave reductions (exact, order-free)
//   - noise per scalefactor band (QuantizePVT.js:725-878): nine consecutive lines per lane, the bands' f64 sums in the
//     reference's line order as a systolic fold over the lanes (f64 sums are order-sensitive, so they are never tree-reduced);
//     the per-band rest (distortion ratio, class, cache) one lane per band
// State (GrInfo scalars) is wave-uniform and lives in registers; spectra and per-band arrays live in LDS.
//
//
// Map of the files.  This file holds no code: every stage is a header of its own, included below in dependency order, each with what it holds.
// Beside them, included by the translation unit: k_quant_tail.h (how a persistent launch ends), k_quant_fast.h (the quality-7 pass) and
// k_quant_probe.h (the test hook over the search's pure functions).
#pragma once
#include "k_quant_prof.h"       // observation scaffolding: PH_* / HO_* profiling macros, the host simulations' counters
#include "k_quant_tabs.h"       // GI, the LDS table image (QuantTabs), the per-wave LDS record (QuantLds), small helpers
#include "k_quant_init.h"       // init_outer_loop, init_xrpow, ordered band sums, calc_xmin and the search limits
#include "k_quant_count.h"      // quantize_xrpow, Huffman region plans, noquant_count_bits / count_bits
#include "k_quant_noise.h"      // calc_noise
#include "k_quant_helper.h"     // count_bits on a helper wave (latency kernels)
#include "k_quant_amp.h"        // scale_bitcount, amplification, balance_noise
#include "k_quant_search.h"     // quant_compare, the bin-search step (bs_advance), the memo flush, bin_search_StepSize + outer_loop (q_outer_loop)
#include "k_quant_framebits.h"  // frame_bits_of, frame_padding (all that k_bits.h needs)
#include "k_quant_finish.h"     // iteration_finish_one: q_best_scalefac_store, q_best_huffman_divide over the per-band Huffman statistics
#include "k_quant_budget.h"     // the seed chain (Seed, seed_before), perceptual entropy and the M/S decision, on_pe / reduce_side: a frame's bit budget
#include "k_quant_frame.h"      // the granule-channel program q_unit and the frame program kb_quant
#include "k_quant_validate.h"   // the seed-chain validation: kb_validate, kb_validate_fast, kb_validate_fast_quad
