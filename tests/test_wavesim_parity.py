"""The wave programs themselves without a GPU: the kernel bodies of lamejs_amd/csrc compiled for the host with NL = 64,
the 64 lanes of a wave running as fibers that meet at every wave primitive (ballots, DPP-style reductions and scans,
lane broadcasts, the systolic folds -- lhip_wave.h, -DLHIP_WAVESIM).  Unlike the one-lane simulation (test_hostsim_parity.py)
this executes exactly the lane-parallel code paths the GPU runs; it is ~20 x slower, hence the smaller cases.  Test-only."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_case_pcm
from libs import WAVESIM_SO, build_sims, wavesim as wsim  # noqa: F401
from oracle_py import oracle_encode

FULL = os.environ.get("LAMEJS_WAVESIM_FULL") == "1"      # the long variant (~4 min): goldens up to 110 frames, 16 random cases


def _encode(lib, ch, kbps, L, R, chunk, sr=44100, joint=False, reservoir=False):
    import lamejs_amd
    enc = lamejs_amd.Mp3Encoder(ch, sr, kbps, lib=lib, joint=joint, reservoir=reservoir)
    out = b""
    for p in range(0, len(L), chunk):
        out += enc.encodeBuffer(L[p:p + chunk], None if R is None else R[p:p + chunk])
    out += enc.flush()
    assert enc.flush() == b""
    enc.close()
    return out


def test_wavesim_matches_small_goldens(wsim, golden):
    """Every golden of at most 40 frames (110 with LAMEJS_WAVESIM_FULL=1): reference output, all sample-rate families."""
    n = 0
    for case in golden:
        if case.get("outside_envelope") or case["corpus"] == "wavfull" or case["nsamples"] > 1152 * (110 if FULL else 40):
            continue
        L, R = load_case_pcm(case)
        mp3 = _encode(wsim, case["channels"], case["kbps"], L, R, case["chunk"], case.get("samplerate", 44100))
        assert hashlib.md5(mp3).hexdigest() == case["mp3_md5"], case
        n += 1
    assert n >= (15 if FULL else 4)


@pytest.mark.parametrize("corpus,ch,sr,kbps,nfr,chunk", [
    ("sine", 1, 44100, 128, 14, 1152 * 14),        # BASELINE config shapes
    ("sine", 2, 44100, 128, 10, 1152 * 3),         # stereo calls of <= 12 frames: the two-waves-per-frame kernel (workgroup barrier)
    ("bursts", 2, 44100, 128, 30, 1152 * 30),      # one larger stereo call: the one-wave-per-frame kernel
    ("bursts", 2, 44100, 320, 24, 4000),           # attacks: short / start / stop blocks, subblock gain
    ("bursts", 1, 48000, 64, 24, 1152 * 24),
    ("bursts", 1, 32000, 192, 24, 777),
    ("bursts", 2, 22050, 64, 24, 1152 * 24),       # MPEG-2: one granule per frame, scale_bitcount_lsf
    ("bursts", 1, 8000, 16, 24, 5000),             # MPEG-2.5
    ("bursts", 1, 48000, 40, 30, 1152 * 30),       # resampled 48 -> 24 kHz in front of the encoder
])
def test_wavesim_matches_oracle(wsim, corpus, ch, sr, kbps, nfr, chunk):
    import pcm
    L, R = pcm.CORPORA[corpus](1152 * nfr + 313, ch, seed=4000 + nfr + kbps)
    got = _encode(wsim, ch, kbps, L, R, chunk, sr)
    assert got == oracle_encode(ch, sr, kbps, L, R)


@pytest.mark.parametrize("corpus,sr,kbps,nfr,chunk", [
    ("centre_bursts", 44100, 128, 14, 1152 * 14),  # M/S frames, one call (the one-wave-per-frame kernel)
    ("bursts", 44100, 128, 24, 1152 * 5),          # M/S and L/R frames mixed; calls of 5 frames: the two-waves-per-frame kernel
    ("centre_sine", 22050, 64, 10, 777),           # MPEG-2
])
def test_wavesim_joint_stereo_matches_oracle(wsim, corpus, sr, kbps, nfr, chunk):
    """SURVEY.md 8f #3 (extension): the 64-lane wave programs in joint-stereo mode against the oracle (itself pinned to the
    reference's joint-stereo output, tests/test_oracle_golden.py)."""
    import pcm
    L, R = pcm.CORPORA[corpus](1152 * nfr, 2)
    got = _encode(wsim, 2, kbps, L, R, chunk, sr, joint=True)
    assert got == oracle_encode(2, sr, kbps, L, R, joint=True)


@pytest.mark.parametrize("corpus,ch,sr,kbps,nfr,chunk,joint", [
    ("bursts", 2, 44100, 128, 16, 1152 * 4, False),
    ("bursts", 1, 22050, 64, 12, 777, False),
    ("centre_bursts", 2, 44100, 128, 10, 1152 * 10, True),      # joint stereo + reservoir: LAME's own default combination
])
def test_wavesim_bit_reservoir_matches_oracle(wsim, corpus, ch, sr, kbps, nfr, chunk, joint):
    """SURVEY.md 8f #4 (extension): the 64-lane wave programs with the bit reservoir in use against the oracle (pinned to the
    reference's reservoir output, tests/test_oracle_golden.py)."""
    import pcm
    L, R = pcm.CORPORA[corpus](1152 * nfr, ch)
    got = _encode(wsim, ch, kbps, L, R, chunk, sr, joint=joint, reservoir=True)
    assert got == oracle_encode(ch, sr, kbps, L, R, joint=joint, reservoir=True)


def test_wavesim_quiet_and_edge_material(wsim):
    """Digital silence, near-silence (analog-silence rule, sparse spectra: the path-dependent table_select leftovers),
    full-scale square wave, and a stream that is shorter than one frame."""
    rng = np.random.default_rng(7)
    n = 1152 * 10
    cases = [np.zeros(n, np.int16), rng.integers(-3, 4, n).astype(np.int16),
             (np.where((np.arange(n) // 40) % 2 == 0, 32767, -32768)).astype(np.int16), rng.integers(-2000, 2000, 700).astype(np.int16)]
    quiet_then_loud = np.concatenate([rng.integers(-2, 3, 1152 * 5), rng.integers(-20000, 20000, 1152 * 5)]).astype(np.int16)
    cases.append(quiet_then_loud)
    for x in cases:
        assert _encode(wsim, 1, 128, x, None, 1152 * 4) == oracle_encode(1, 44100, 128, x)
    assert _encode(wsim, 2, 128, cases[1], cases[4][:n], 3000) == oracle_encode(2, 44100, 128, cases[1], cases[4][:n])


def test_wavesim_seed_repair_path(wsim):
    """Poor speculative bin-search seed: validation (memo replay with ballots / lane broadcasts) flags frames, the repair
    passes converge to the reference's bytes."""
    import lamejs_amd, pcm
    L, R = pcm.bursts(1152 * 10, 2, seed=77)
    want = oracle_encode(2, 44100, 128, L, R)
    try:
        assert wsim.lhip_debug_set_spec_seed(255, 1) == 0
        enc = lamejs_amd.Mp3Encoder(2, 44100, 128, lib=wsim)
        got = enc.encodeBuffer(L, R)
        stats = enc.last_batch_stats()
        got += enc.flush()
        assert stats["repaired_frames"] > 0, stats
        assert got == want
    finally:
        wsim.lhip_debug_set_spec_seed(180, 4)


def test_wavesim_batch_streams(wsim):
    import lamejs_amd, pcm
    streams = [pcm.bursts(1152 * (4 + i), 1, seed=2000 + i)[0] for i in range(3)]
    encs = [lamejs_amd.Mp3Encoder(1, 44100, 128, lib=wsim) for _ in streams]
    got = lamejs_amd.encode_streams(encs, streams)
    for s, g in zip(streams, got):
        assert g == oracle_encode(1, 44100, 128, s)


def test_wavesim_random_material(wsim):
    """A short sweep of the seeded random material the GPU fuzz uses (tones, coloured noise, clicks, silence gaps, level
    steps) over MPEG-1, MPEG-2/2.5 and resampling configurations."""
    import sys
    sys.path.insert(0, str(ROOT / "tests" / "tools"))
    import fuzz_gpu
    n1, n2, n3 = (6, 6, 4) if FULL else (2, 2, 1)
    assert fuzz_gpu.run(n1, 2024, lib=wsim, verbose=False) == []
    assert fuzz_gpu.run(n2, 31, lib=wsim, verbose=False, cfgs=fuzz_gpu.LSF_CFGS) == []
    assert fuzz_gpu.run(n3, 5, lib=wsim, verbose=False, cfgs=fuzz_gpu.RESAMPLE_CFGS) == []


def test_wavesim_ath_scan_segments(wsim):
    """The ATH recurrence as the device runs it -- a workgroup whose threads own segments of frames, evaluate them from their first
    reset point and fill in the prefixes round by round once the previous segment's end state is known (k_psy_scan.h kb_scan_ath).  The
    one-lane simulation runs it with one thread; here it is a two-wave workgroup (128 threads, two-frame segments, 256-frame chunks),
    so 600 frames of quiet noise with bursts walk through three chunks, multi-frame segments, resets, prefix rounds and the chunk
    carry.  ATH.adjust of every frame (and every other stage tap) against the oracle."""
    import pcm, stage_taps
    L, _ = pcm.bursts(1152 * 600, 1, seed=5)
    assert stage_taps.compare_stages(wsim, 1, 44100, 128, L, None) == []


def test_wavesim_tail_help():
    """How a launch of the persistent quantization kernel ends (csrc/k_quant_tail.h; the shipped g_quant since round 4): the kernel as a
    real 8-wave workgroup in which waves that find the frame dispenser empty quantize the second channel of granules their neighbours
    are working on.  Two-channel cases in one batch each (plain, joint stereo, MPEG-2) against the oracle,
    and both ways of an offer -- taken by a helper, withdrawn by its owner -- must have been exercised."""
    import sys
    build_sims()
    code = ("import sys; sys.path.insert(0, r'%s'); sys.path.insert(0, r'%s'); sys.path.insert(0, r'%s'); import lamejs_amd, fuzz_gpu\n"
            "lib = lamejs_amd.load_library(r'%s')\n"
            "bad = fuzz_gpu.run(5, 4401, lib=lib, verbose=False, stereo_only=True, whole=True, max_frames=40)\n"
            "bad += fuzz_gpu.run(4, 4402, lib=lib, verbose=False, joint=True, whole=True, max_frames=40)\n"
            "bad += fuzz_gpu.run(4, 4403, lib=lib, verbose=False, cfgs=fuzz_gpu.LSF_CFGS, stereo_only=True, whole=True, max_frames=40)\n"
            "print('BAD', bad)\n") % (ROOT, ROOT / "tests", ROOT / "tests" / "tools", WAVESIM_SO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, LAMEJS_TAILHELP_STATS="1"), timeout=900)
    assert r.returncode == 0 and "BAD []" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])
    import re
    m = re.search(r"tail-help: (\d+) granule-channels by helpers, (\d+) offers withdrawn", r.stderr)
    assert m and int(m.group(1)) > 10 and int(m.group(2)) > 10, r.stderr[-500:]


def test_wavesim_one_frame_launch_count_helpers():
    """The one-frame launch as a real eight-wave workgroup (csrc/k_frame.h kb_frame_stage, k_quant_helper.h q_count_helper / q_count_bits_piped; round 5): 1152
    samples per call -- the reference's documented call pattern -- on one- and two-channel streams, MPEG-1 and MPEG-2, joint stereo and the bit reservoir
    (whose multi-frame calls run the per-stream kernel with the same helpers).  Every call's bytes against the oracle, and both fates of a calc_noise made
    beside the helper's count -- committed, dropped because the evaluation did not fit -- must have occurred; so must a one-channel frame's wait for the
    psyB wave (MPEG-1 mono) and the two-channel barrier path."""
    import sys
    build_sims()
    code = ("import sys; sys.path.insert(0, r'%s'); sys.path.insert(0, r'%s'); sys.path.insert(0, r'%s'); import numpy as np, lamejs_amd, fuzz_gpu\n"
            "from oracle_py import oracle_encode\n"
            "lib = lamejs_amd.load_library(r'%s')\n"
            "rng = np.random.default_rng(5150); bad = []\n"
            "for (ch, sr, kb, joint, resv, chunk) in ((2, 44100, 128, False, False, 1152), (1, 44100, 128, False, False, 1152), (2, 22050, 64, False, False, 576), (1, 16000, 32, False, False, 576),\n"
            "                                       (2, 44100, 128, True, False, 1152), (2, 44100, 192, False, True, 1152), (1, 44100, 64, False, True, 4000)):\n"
            "    L, R = fuzz_gpu.material(rng, 1152 * 9 + 301, ch)\n"
            "    enc = lamejs_amd.Mp3Encoder(ch, sr, kb, lib=lib, joint=joint, reservoir=resv)\n"
            "    got = b''.join(enc.encodeBuffer(L[p:p + chunk], None if R is None else R[p:p + chunk]) for p in range(0, len(L), chunk)) + enc.flush()\n"
            "    if got != oracle_encode(ch, sr, kb, L, R, joint=joint, reservoir=resv): bad.append((ch, sr, kb, joint, resv))\n"
            "print('BAD', bad)\n") % (ROOT, ROOT / "tests", ROOT / "tests" / "tools", WAVESIM_SO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=dict(os.environ, LAMEJS_PIPE_STATS="1"), timeout=900)
    assert r.returncode == 0 and "BAD []" in r.stdout, (r.stdout[-800:], r.stderr[-1500:])
    import re
    m = re.search(r"count helper: (\d+) evaluations counted on the helper wave, (\d+) of the calc_noise calls made beside them committed", r.stderr)
    assert m and int(m.group(2)) > 100 and int(m.group(1)) - int(m.group(2)) > 100, r.stderr[-500:]


@pytest.mark.parametrize("ch,nstreams", [(1, 3), (2, 2)])
def test_wavesim_one_frame_batch_of_streams(wsim, ch, nstreams):
    """`encodeBatch` over several streams fed 1152 samples per call: the eight-wave one-frame launch once per stream of the batch.  (Round 5's
    simulation set the count helpers' records to idle once per batch instead of once per workgroup and hung on the second stream; the device
    kernel initialises them per workgroup.)"""
    import lamejs_amd, pcm
    mats = [pcm.bursts(1152 * 4 + 100 * i, ch, seed=3100 + 10 * ch + i) for i in range(nstreams)]
    encs = [lamejs_amd.Mp3Encoder(ch, 44100, 128, lib=wsim) for _ in mats]
    got = [b""] * nstreams
    n = max(len(m[0]) for m in mats)
    for p in range(0, n, 1152):
        outs = lamejs_amd.encode_streams(encs, [m[0][p:p + 1152] for m in mats], None if ch == 1 else [m[1][p:p + 1152] for m in mats], flush=False)
        got = [g + o for g, o in zip(got, outs)]
    got = [g + e.flush() for g, e in zip(got, encs)]
    for m, g in zip(mats, got):
        assert g == oracle_encode(ch, 44100, 128, m[0], m[1])


def test_wavesim_interleaved_live_encoders(wsim):
    """The interleaved live encoders of tests/interleaved.py on the 64-lane simulation (eight-wave one-frame launches of different configurations
    in turn: g_frame<0> / g_frame<1>, count helpers on and off), a shorter run."""
    import interleaved
    assert interleaved.run(wsim, 606062, nframes=6) == []
