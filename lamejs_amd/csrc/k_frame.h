// k_frame.h -- the two programs that take a stream through all stages inside one launch: kb_frame_stage (one frame per stream) and
// kb_resv_stage (bit reservoir: all frames of a stream).
// Part of lhip_api.cpp's one translation unit (included there, in the order the definitions need).
#pragma once
// ===========================================================================================
// One frame per stream in ONE launch (small batches: the drop-in's own 1152-sample call pattern, and every launch of the bit-reservoir
// mode).  A batch of one frame per stream is a chain of thirteen tiny kernels otherwise, each waiting for the one before it: the
// gaps between dependent launches cost as much as the frame's quantization.  Here a workgroup of FR_WAVES waves takes a stream
// through all stages, a workgroup barrier between them; every stage is the same kb_* body the separate kernels run, so the bytes
// cannot differ.  The LDS of a wave is a union of the stages' structures.
// ===========================================================================================
// Stages of the frame program (workgroup barriers in between).  Stages that do not depend on each other share a slot on different waves
// (round 5: the launch's critical path is  load | psyA | scans | psyB | quantization | bit packing;  the polyphase filterbank runs beside
// psyA, the MDCT beside psyB, the state save beside the bit packing -- profiles/r05_pass1_frame_prof_*.txt has the stage times this is
// built on).  FR_WAVES waves per workgroup whatever the channel mode.
enum { FS_LOAD, FS_PREP, FS_PSYA_POLY, FS_PSYA_MS, FS_SCAN_RAW, FS_SCAN_ATTACK, FS_SCAN_BT, FS_PSYB0_MDCT, FS_PSYB1, FS_QUANT, FS_BITS_SAVE,
       FR_STAGES, FR_WAVES = 8, FR_LDS_PER_WAVE = (sizeof(PolyLds) + 15) & ~15 };
static_assert(sizeof(PsyALds) <= FR_LDS_PER_WAVE && sizeof(PsyBLds4) <= FR_LDS_PER_WAVE && sizeof(MdctLds) <= FR_LDS_PER_WAVE &&
              sizeof(QuantLds) <= FR_LDS_PER_WAVE && sizeof(BitsLds) <= FR_LDS_PER_WAVE, "frame kernel: the per-wave LDS union is sized by PolyLds");
// a stage nobody has work in for this configuration (wave-uniform: a function of the tables and the instantiation) -- skipped with its barrier
template <int RESV> LHIP_DEV bool frame_stage_empty(int stage, const Tables& T) {
    return (stage == FS_PREP && T.rs_ratio == 1) || (stage == FS_PSYA_MS && T.psy_channels != 4) || stage == FS_PSYB1 ||
           ((stage == FS_SCAN_RAW || stage == FS_SCAN_ATTACK) && !RESV && T.mode != 1);      // (the flow of kb_frame_stage runs these two scans inside FS_PSYA_POLY)
}
// What a one-frame launch does BESIDE the search of the frame's first granule (FS_QUANT, waves 4 .. 7; no reservoir, no joint stereo): wave 4 + j holds the
// energies of (granule, channel) pair j in its LDS (kb_psyA<3>, FS_PSYA_POLY) and finishes that pair's psyA (partitions, tonality, short spreading); when both
// channels of a granule are done the first channel's wave runs the granule's psyB.  The second granule's filterbank and MDCT follow on waves that are free by then
// (two channels: 5 and 7 after their psyA parts; one channel: 6).  Meeting points are counters in LDS among the waves concerned (wg_meet; mbox[6 ..], zeroed in
// FS_PSYB0_MDCT).  The second granule's search needs psyB(granule 0) and its own MDCT: a two-channel frame's waves arrive at the workgroup barrier between the
// granules only after all of this; a one-channel frame's second granule waits for mbox[3], set here once both are done.
LHIP_DEV void frame_flow_tail(const Tables& T, const PowBase& pb, const Workspace& W, const StreamDesc* SD, const StreamIO* IO, int g1, int wv, int lane,
                         unsigned char* lds, int* mbox) {
    const int C = T.channels_out, GR = T.mode_gr, np = GR * C, j = wv - 4;
    if (j >= 0 && j < np) {
        const int g = j / C;
        kb_psyA<4>(T, W, SD, IO, g1 + g, j % C, lane, *(PsyALds*)lds);
        if (C == 2) wg_meet(mbox + 6 + g, 2, lane);
        wave_sync();                                          // (the wave's LDS changes its meaning)
        if (j % C == 0) kb_psyB<4>(T, pb, W, SD, g1 + g, lane, *(PsyBLds4*)lds, -1, 0, 0);
    }
    if (GR == 2) {
        const bool fb = C == 2 ? (wv == 5 || wv == 7) : wv == 6;      // the second granule's filterbank: channel 0 on wave 5 (6), channel 1 on wave 7
        if (fb) {
            wave_sync();
            kb_poly_run(T, W, SD, IO, g1 + 1, C == 2 ? (wv - 5) / 2 : 0, 1, lane, *(PolyLds*)lds);
            if (C == 2) wg_meet(mbox + 8, 2, lane);
            wave_sync();
            if (wv != 7) kb_mdct(T, W, SD, g1 + 1, lane, *(MdctLds*)lds);
        }
        if (C == 1 && (wv == 4 || wv == 6)) {
            wg_meet(mbox + 9, 2, lane);
            if (wv == 4) wg_store(mbox + 3, 1, lane);
        }
    }
}
// stage `stage` of the frame program for wave `wv` (of `nw` >= 6) of the workgroup that owns stream `st`.  PAIRQ: stereo quantization by
// two waves (kb_quant<1>, which meets once per granule at a workgroup barrier: the other waves keep the barrier count).
template <int RESV, int PAIRQ>
LHIP_DEV void kb_frame_stage(int stage, const Tables& T, const PowBase& pb, const Workspace& W, const StreamDesc* SD, const StreamIO* IO,
                             int st, int wv, int nw, int lane, unsigned char* lds, QuantTabs& Q, int* mbox, CountShare* cshare = nullptr) {
    const int C = T.channels_out, Cp = T.psy_channels, GR = T.mode_gr;
    const StreamDesc sd = SD[st];
    const bool has = sd.nframes > 0;                          // this launch completes a frame of the stream (else only the state moves)
    const int g1 = sd.gslot0 + 1, fslot = sd.fslot0 + 1;
    ResvState* rv = RESV ? &IO[st].state->rv : nullptr;       // one-frame launches work on the record in global memory
    const int side0 = nw - 2;                                 // the two waves that run the filterbank beside the psychoacoustics
    const bool psyb_late = !RESV && T.mode != 1;              // psyB beside the quantization of granule 0 (FS_QUANT) instead of in front of it
    const bool flow = PAIRQ && psyb_late && nw == 8;          // ... and with it everything else the first granule's search does not need (frame_flow_tail)
    switch (stage) {
        case FS_LOAD: kb_load(T, W, SD, IO, st, lane, wv, nw); if (wv == 0 && lane == 0) mbox[10] = 0; break;      // ([10]: FS_PSYA_POLY's meeting point)
        case FS_PREP: if (T.rs_ratio != 1) kb_prep_stream(T, W, SD, IO, st, (int64_t)wv * LHIP_NL + lane, (int64_t)nw * LHIP_NL); break;
        case FS_PSYA_POLY:
            // Without the reservoir and outside joint stereo (psyb_late) only what the search of the frame's FIRST granule needs stays in front of it:
            //   here      waves 4 + j: pair j's spectra up to the loudness (kb_psyA<3>);  waves 0 (1): granule 0's filterbank;  waves 2, 3: the high-passes
            //   FS_SCAN_* wave 0;   FS_PSYB0_MDCT  wave 1: granule 0's MDCT
            //   FS_QUANT  beside the search (frame_flow_tail): psyA's partitions / tonality (kb_psyA<4>, on the waves that hold the energies) -> psyB; the
            //             second granule's filterbank -> its MDCT, which the second granule's search waits for
            // (measured: a polyphase granule is 17 us of ONE lane's arithmetic whatever else the wave does, psyA's tail 8.7 us: 25.7 -> 17 us for this stage)
            if (flow) {
                const int np = GR * C;
                if (!has) break;
                if (wv >= 4 && wv - 4 < np) kb_psyA<3>(T, W, SD, IO, g1 + (wv - 4) / C, (wv - 4) % C, lane, *(PsyALds*)lds);
                else if (wv < C) kb_poly_run(T, W, SD, IO, g1, wv, 1, lane, *(PolyLds*)lds);
                else if (wv == 2 || wv == 3) {
                    for (int j = wv - 2; j < np; j += 2) { kb_psyA<1>(T, W, SD, IO, g1 + j / C, j % C, lane, *(PsyALds*)lds); wave_sync(); }
                    // the first two scans (attack flags from the peaks) right behind the high-passes, well inside the stage: FS_SCAN_RAW / _ATTACK are empty then
                    wg_meet(mbox + 10, 2, lane);
                    if (wv == 2) {
                        for (int g = lane; g < GR; g += LHIP_NL) kb_scan_raw(T, W, SD, g1 + g);
                        wave_sync_global();
                        for (int g = lane; g < GR; g += LHIP_NL) kb_scan_attack(T, W, SD, g1 + g);
                    }
                }
                break;
            }
            // One-frame launches on the device: waves [0, GR C) take the spectra and everything after them (kb_psyA<2>, the stage's longest chain); wave GR C + j
            // takes (granule, channel) pair j's polyphase filterbank and then its high-pass + sub-block peaks (kb_psyA<1>: a fifth of psyA, needed by the scans
            // only) -- on one wave per channel the filterbank of both granules was as long as all of psyA
            if (PAIRQ && nw >= 2 * GR * C) {
                const int np = GR * C;
                if (has && wv < np) kb_psyA<2>(T, W, SD, IO, g1 + wv / C, wv % C, lane, *(PsyALds*)lds);
                else if (has && wv < 2 * np) {
                    const int j = wv - np;
                    kb_poly_run(T, W, SD, IO, g1 + j / C, j % C, 1, lane, *(PolyLds*)lds);
                    wave_sync();                                  // (the wave's LDS changes its meaning)
                    kb_psyA<1>(T, W, SD, IO, g1 + j / C, j % C, lane, *(PsyALds*)lds);
                }
                break;
            }
            if (has && wv < GR * C) kb_psyA(T, W, SD, IO, g1 + wv / C, wv % C, lane, *(PsyALds*)lds);
            else if (has && wv >= side0 && wv - side0 < C) kb_poly_run(T, W, SD, IO, g1, wv - side0, GR, lane, *(PolyLds*)lds);
            break;
        case FS_PSYA_MS: if (has && Cp == 4 && wv < GR * 2) kb_psyA(T, W, SD, IO, g1 + wv / 2, 2 + wv % 2, lane, *(PsyALds*)lds); break;
        case FS_SCAN_RAW: if (!flow && has && wv == 0) for (int g = lane; g < GR; g += LHIP_NL) kb_scan_raw(T, W, SD, g1 + g); break;
        case FS_SCAN_ATTACK: if (!flow && has && wv == 0) for (int g = lane; g < GR; g += LHIP_NL) kb_scan_attack(T, W, SD, g1 + g); break;
        case FS_SCAN_BT:
            if (has && wv == 0) {
                for (int g = lane; g < GR; g += LHIP_NL) kb_scan_blocktype(T, W, SD, g1 + g);
                if (lane == 0) {                              // adjust_ATH of the one frame (Encoder.js:166-243)
                    double a = W.ath_adjust[sd.fslot0], l = W.ath_limit[sd.fslot0];
                    ath_step(T, ath_max_pow(T, W, sd, C, 0), a, l);
                    W.ath_adjust[fslot] = a; W.ath_limit[fslot] = l;
                }
            }
            break;
        case FS_PSYB0_MDCT:   // the MDCT needs the block types (scans) and the polyphase output.  Bit reservoir: psyB here too, the frame's granules one after
                              // the other (FS_PSYB1 takes the second) -- their thresholds depend on the reservoir; joint stereo: psyB here as well (the frame's M/S
                              // decision reads granule 0's thresholds before anything is quantized); otherwise psyB runs beside the quantization (psyb_late)
            if (flow) { if (has && wv == 1) kb_mdct(T, W, SD, g1, lane, *(MdctLds*)lds); }       // granule 0 only (waves 4 .. 7 keep psyA's energies in their LDS)
            else if (has && !psyb_late && (RESV ? wv == 0 : wv < GR)) kb_psyB<4>(T, pb, W, SD, g1 + (RESV ? 0 : wv), lane, *(PsyBLds4*)lds, -1, RESV ? rv->ResvSize : 0, RESV ? rv->ResvMax : 0);
            else if (has && wv >= side0 && wv - side0 < GR) kb_mdct(T, W, SD, g1 + (wv - side0), lane, *(MdctLds*)lds);
            if (wv == 0 && lane == 0) for (int i = 0; i < 12; i++) mbox[i] = 0;     // [3] "granule 1 may be searched" (FS_QUANT, one-channel frames); [4], [5] the bit packers' meeting points (FS_BITS_SAVE); [6 ..] frame_flow_tail's
            break;
        case FS_PSYB1: break;     // (the reservoir's second psyB runs beside the quantization now: FS_QUANT)
        case FS_QUANT:
            // waves 0 (1): the channel's search; waves 2 (3): its count helper (q_count_helper: the Huffman count of an evaluation while the owner
            // runs calc_noise); the one-lane simulation (PAIRQ == 0) has neither
            // Without the reservoir (and outside joint stereo) psyB is not on the frame's critical path: granule 0 is quantized against the thresholds the PREVIOUS call left
            // (the carry slot), granule 1 against psyB(granule 0)'s, and psyB(granule 1)'s are only saved for the next call.  Waves 4 (5) run psyB
            // while granule 0 is quantized; a two-channel frame's granules are separated by a workgroup barrier anyway (the channels exchange their
            // bits), a one-channel frame's second granule waits for mbox[3].  The one-lane simulation (PAIRQ == 0, waves one after the other) runs
            // psyB first.
            if (!PAIRQ && psyb_late && has && wv == 0) for (int g = 0; g < GR; g++) kb_psyB<4>(T, pb, W, SD, g1 + g, lane, *(PsyBLds4*)lds, -1, 0, 0);
            // Bit reservoir: psyB of the SECOND granule beside the quantization, on wave 4 -- nothing of this frame reads what it leaves (granule 1 is quantized against
            // psyB(granule 0)'s thresholds, the frame's entropies are those of the maskings in use), the next call does (kb_resv_stage, RS_QUANT: the same)
            if (RESV && GR == 2 && has && wv == 4) kb_psyB<4>(T, pb, W, SD, g1 + 1, lane, *(PsyBLds4*)lds, -1, rv->ResvSize, rv->ResvMax);
            if (PAIRQ && C == 2) {
                if (has && wv < 2) {
                    kb_quant<1, RESV>(T, pb, W, SD, fslot, RESV ? 2 : 0, lane, *(QuantLds*)lds, Q, wv, mbox, rv, nullptr, cshare ? cshare + wv : nullptr);
                    if (cshare) wg_store(&cshare[wv].state, CS_QUIT, lane);
                }
#if LHIP_NL != 1
                else if (has && cshare && wv < 4) q_count_helper(T, cshare[wv - 2], *(const QuantLds*)(lds - 2 * FR_LDS_PER_WAVE), *(QuantLds*)lds, Q, lane);
#endif
                else {
                    if (flow && has) frame_flow_tail(T, pb, W, SD, IO, g1, wv, lane, lds, mbox);
                    else if (psyb_late && has && wv >= 4 && wv - 4 < GR) kb_psyB<4>(T, pb, W, SD, g1 + (wv - 4), lane, *(PsyBLds4*)lds, -1, 0, 0);
                    for (int gr = 0; gr < GR; gr++) wg_barrier();
                }
            } else if (has && wv == 0) {
                kb_quant<0, RESV>(T, pb, W, SD, fslot, RESV ? 2 : 0, lane, *(QuantLds*)lds, Q, -1, nullptr, rv, nullptr, PAIRQ ? cshare : nullptr, (PAIRQ && psyb_late) ? mbox + 3 : nullptr);
                if (PAIRQ && cshare) wg_store(&cshare[0].state, CS_QUIT, lane);
            }
#if LHIP_NL != 1
            else if (PAIRQ && has && cshare && wv == 2) q_count_helper(T, cshare[0], *(const QuantLds*)(lds - 2 * FR_LDS_PER_WAVE), *(QuantLds*)lds, Q, lane);
#endif
            else if (flow && has && wv >= 4) frame_flow_tail(T, pb, W, SD, IO, g1, wv, lane, lds, mbox);      // (sets the flag granule 1 waits for)
            else if (PAIRQ && psyb_late && has && wv == 4) {           // one-channel frame: both granules' psyB on this wave, then the flag granule 1 waits for
                for (int g = 0; g < GR; g++) kb_psyB<4>(T, pb, W, SD, g1 + g, lane, *(PsyBLds4*)lds, -1, 0, 0);
                wg_store(mbox + 3, 1, lane);
            }
            break;
        case FS_BITS_SAVE:   // the state record's reservoir part belongs to the bit packer, everything else to the save: disjoint words
            if (PAIRQ && !RESV && nw > GR * C) {
                // no reservoir: a frame's granule-channels are packed side by side by waves [0, GR C) into wave 0's frame image (kb_bits_mw), the other
                // waves save the state
                const int nb = GR * C;
                uint32_t* wsh = ((BitsLds*)(lds - (size_t)wv * FR_LDS_PER_WAVE))->w;
                if (wv >= nb) kb_save(T, W, SD, IO, st, lane, wv - nb, nw - nb);
                else if (has) kb_bits_mw(T, W, SD, fslot, lane, *(BitsLds*)lds, wsh, wv, nb, mbox + 4);
                break;
            }
            if (wv == 0) { if (has) kb_bits(T, W, SD, fslot, lane, *(BitsLds*)lds, rv, W.out_bytes + st); }
            else kb_save(T, W, SD, IO, st, lane, wv - 1, nw - 1);
            break;
        default: break;
    }
}

// ===========================================================================================
// Bit reservoir: ALL frames of a stream in one launch.  With the reservoir in use a frame's bit budget and -- through pcfact -- the
// second half of its psychoacoustics depend on the bits every earlier frame spent: the frames of a stream are a
// serial chain.  What does NOT depend on the reservoir (load, resampling, psyA, the scans, the ATH recurrence, polyphase, MDCT) runs
// batched over all frames of all streams like any other batch; then ONE workgroup per stream walks the stream's frames in order:
//     psyB(granule 0) | quantization        (a workgroup barrier after each)
// with the stream's reservoir record in LDS for the whole walk, the bit packing of frame k - 1 beside psyB(granule 0) of frame k on another
// wave (the packer commits the record; psyB takes the reservoir fill from what the quantization of frame k - 1 decided, W.fr, so the two do
// not touch the same words), and psyB(granule 1) beside the quantization (only the NEXT frame reads what it leaves; round 5: it was a stage of
// its own, 11 us of a frame's 183).  No launch and no read-back per frame: the byte counts stay on the device until the call ends.
// Waves: 0 (and 1: second channel, kb_quant<1>) quantize, 2 runs psyB, 3 packs bits.
// ===========================================================================================
enum { RS_PSYB0, RS_QUANT, RS_STAGES, RS_WAVES = 4,
       RS_LDS_PER_WAVE = ((sizeof(QuantLds) > sizeof(PsyBLds4) ? (sizeof(QuantLds) > sizeof(BitsLds) ? sizeof(QuantLds) : sizeof(BitsLds))
                                                                : (sizeof(PsyBLds4) > sizeof(BitsLds) ? sizeof(PsyBLds4) : sizeof(BitsLds))) + 15) & ~15 };
// stage `stage` of frame k (of F) of stream st for wave wv; k == F: only the tail (bit packing of the last frame)
// cshare (device, wave simulation): the count helpers' records -- while a frame is quantized the psyB and the bit-packing wave have nothing to do
// and take the Huffman counts of waves 0 / 1 (q_count_helper, k_quant_helper.h)
template <int PAIRQ>
LHIP_DEV void kb_resv_stage(int stage, const Tables& T, const PowBase& pb, const Workspace& W, const StreamDesc* SD, int st, int k, int F,
                            int wv, int lane, unsigned char* lds, QuantTabs& Q, int* mbox, ResvState& RV, int32_t* nout, CountShare* cshare = nullptr) {
    const int C = T.channels_out, GR = T.mode_gr;
    const StreamDesc sd = SD[st];
    const int g1 = sd.gslot0 + 1 + GR * k, fslot = sd.fslot0 + 1 + k, fidx = sd.out_slot0 + k;
    switch (stage) {
        case RS_PSYB0:
            if (cshare && wv < 2 && lane == 0) cshare[wv].state = CS_IDLE;      // (the helpers look at it one barrier from here)
            if (wv == 2 && k < F) {       // the reservoir as frame k - 1 left it: decided by that frame's quantization (the packer may still be committing it)
                const int rs = k == 0 ? RV.ResvSize : W.fr[fidx - 1].ResvSize, rm = k == 0 ? RV.ResvMax : W.fr[fidx - 1].ResvMax;
                kb_psyB<4>(T, pb, W, SD, g1, lane, *(PsyBLds4*)lds, -1, rs, rm);
            }
            if (wv == 3 && k > 0) kb_bits(T, W, SD, fslot - 1, lane, *(BitsLds*)lds, &RV, nout);
            break;
        case RS_QUANT:
            if (k >= F) break;
            // psyB of the frame's SECOND granule runs beside the quantization: nothing of frame k reads what it leaves (the psychoacoustics are one
            // granule ahead of their use: granule 1 is quantized against psyB(granule 0)'s thresholds, and the frame's entropies -- q_frame_pe -- are
            // those of the maskings in use), frame k + 1 does, two barriers from here.  Two-channel frames: on wave 2 before it turns count helper (the
            // searches post their first request after their bin searches, which take longer than this); one-channel frames: on wave 3, which has nothing else to do.
            if (GR == 2 && ((PAIRQ && wv == (C == 2 ? 2 : 3)) || (!PAIRQ && wv == 2))) {
                const int rs = k == 0 ? RV.ResvSize : W.fr[fidx - 1].ResvSize, rm = k == 0 ? RV.ResvMax : W.fr[fidx - 1].ResvMax;
                kb_psyB<4>(T, pb, W, SD, g1 + 1, lane, *(PsyBLds4*)lds, -1, rs, rm);
            }
            if (PAIRQ && C == 2) {
                if (wv < 2) { kb_quant<1, 1>(T, pb, W, SD, fslot, 2, lane, *(QuantLds*)lds, Q, wv, mbox, &RV, nullptr, cshare ? cshare + wv : nullptr); if (cshare) wg_store(&cshare[wv].state, CS_QUIT, lane); }
#if LHIP_NL != 1
                else if (cshare) q_count_helper(T, cshare[wv - 2], *(const QuantLds*)(lds - 2 * RS_LDS_PER_WAVE), *(QuantLds*)lds, Q, lane);
#endif
                else for (int gr = 0; gr < GR; gr++) wg_barrier();
            } else if (wv == 0) { kb_quant<0, 1>(T, pb, W, SD, fslot, 2, lane, *(QuantLds*)lds, Q, -1, nullptr, &RV, nullptr, PAIRQ ? cshare : nullptr); if (PAIRQ && cshare) wg_store(&cshare[0].state, CS_QUIT, lane); }
#if LHIP_NL != 1
            else if (PAIRQ && cshare && wv == 2) q_count_helper(T, cshare[0], *(const QuantLds*)(lds - 2 * RS_LDS_PER_WAVE), *(QuantLds*)lds, Q, lane);
#endif
            break;
        default: break;
    }
}
